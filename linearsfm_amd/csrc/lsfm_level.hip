// The level driver: the camera systems of one tree level from the joint maps to the solved poses and features (solve_batch).
//   * a level of small systems (small_level_strips, lsfm_small.hip) is one launch: solve_level_dense;
//   * any other level runs the sparse pipeline: its structure -- pattern of S, Schur assembly K9, symbolic factorisation -- from
//     wherever the level gets it (level_structure: a recorded plan, a plan or a pattern prepared one level ahead, a pattern built
//     early or beside the right-hand sides, or in line), then the refinement's set-up (lsfm_pcg.hip), the numeric factorisation
//     (lsfm_chol.hip), the refinement, the back-substitution (lsfm_solve.hip) and the level's outcome;
//   * what a first solve of a level leaves for the next runs of the same tree (SolvePlan), and what is prepared for the NEXT level
//     on a side stream and the helper thread while the device works on this one (PreLevel, prefetch_next_level);
//   * the debug / test modes of a level: LSFM_FACTOR_DIGEST, LSFM_CHECK_EARLY_PATTERN, LSFM_DEBUG, LSFM_DEBUG_CONV.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "lsfm_device.hpp"
#include "lsfm_symbolic.hpp"
#include "lsfm_pcg.hpp"

namespace lsfm {

// What a first solve of a tree level leaves for the next runs of the same tree (LevelPlan::solve): the block pattern of S
// with its hash index and the whole symbolic factorisation, in one device allocation of their own.
struct SolvePlan {
	SchurSystem sy; // index members only (S, E, IV are per run)
	CholDev ch;     // index members + host vectors (L, Lg, Dinv, d_err are per run)
	int its = 1;    // refinement steps the first run needed ...
	bool mixed = false; // ... with the preconditioner in this precision
	double rel_tol = 0; // ... to this relative residual
	bool small = false; // the plan of a level on the one-launch dense path: no pattern, no factorisation (lsfm_small.hip)
	char* mem = nullptr;
	~SolvePlan() { if (mem) (void)hipFree(mem); }
};
static std::shared_ptr<SolvePlan> solve_plan_store(lsfm_context* ctx, const SchurSystem& sy, const CholDev& ch, int its)
{
	auto sp = std::make_shared<SolvePlan>();
	const size_t M = sy.M, nnzb = sy.nnzb, cap = (size_t)sy.mask + 1;
	if (getenv("LSFM_DEBUG") && sy.k9.ns && sy.k9_tiles > 0)
	{
		// census of the Schur tiles by the number of poses that see them (negative: no panel variant took the tile)
		std::vector<int> h(sy.k9_tiles);
		d2h(ctx, h.data(), sy.k9.ns, sizeof(int) * h.size());
		int b16 = 0, b32 = 0, b48 = 0, b64 = 0, b96 = 0, more = 0;
		for (int v : h) { const int n = v < 0 ? -v : v; (n <= 16 ? b16 : n <= 32 ? b32 : n <= 48 ? b48 : n <= 64 ? b64 : n <= 96 ? b96 : more)++; }
		fprintf(stderr, "[lsfm] Schur tiles by poses: <=16 %d, <=32 %d, <=48 %d, <=64 %d, <=96 %d, more (or > 64 distinct: hash full) %d\n", b16, b32, b48, b64, b96, more);
	}
	struct Item { const void* src; size_t bytes; void** dst; };
	SolvePlan& P = *sp;
	P.sy = sy; P.ch = ch; P.its = its; P.mixed = ch.Lf != nullptr; P.rel_tol = ctx->pcg.rel_tol;
	P.sy.S = nullptr; P.sy.E = nullptr; P.sy.IV = nullptr;
	P.ch.L = nullptr; P.ch.Dinv = nullptr; P.ch.diag0 = nullptr; P.ch.dscale = nullptr; P.ch.Lg = nullptr; P.ch.Lgf = nullptr; P.ch.d_err = nullptr; P.ch.wv = nullptr; P.ch.Lf = nullptr; P.ch.Dinvf = nullptr;
	std::vector<Item> items = {
		{ sy.rowptr, (M + 1) * 4, (void**)&P.sy.rowptr }, { sy.colidx, (nnzb + 1) * 4, (void**)&P.sy.colidx },
		{ sy.upper_keys, nnzb * 8, (void**)&P.sy.upper_keys }, { sy.longrows, (M + 1) * 4, (void**)&P.sy.longrows },
		{ sy.d_nlong, 4, (void**)&P.sy.d_nlong }, { sy.tab, cap * 8, (void**)&P.sy.tab }, { sy.hval, cap * 4, (void**)&P.sy.hval },
		{ ch.blob, ch.blob_ints * 4, (void**)&P.ch.blob },
		{ sy.gent, sy.gent ? nnzb * 16 : 0, (void**)&P.sy.gent }, { sy.goth, sy.goth ? nnzb * 8 : 0, (void**)&P.sy.goth },
		{ sy.k9.ns, sy.k9.ns ? (size_t)sy.k9_tiles * 4 : 0, (void**)&P.sy.k9.ns }, { sy.k9.pose, sy.k9.pose ? (size_t)sy.k9_tiles * 64 * 4 : 0, (void**)&P.sy.k9.pose },
		{ sy.k9.eslot, sy.k9.eslot ? (size_t)sy.k9_NW : 0, (void**)&P.sy.k9.eslot },
		{ sy.k9.wlist, sy.k9.wlist ? (size_t)sy.k9_tiles * 3 * 4 : 0, (void**)&P.sy.k9.wlist }, { sy.k9.wcnt, sy.k9.wcnt ? (size_t)32 : (size_t)0, (void**)&P.sy.k9.wcnt },
	};
	size_t total = 0;
	for (const Item& it : items) total += (it.bytes + 255) & ~(size_t)255;
	LSFM_CHECK_HIP(hipMalloc((void**)&P.mem, total + 256));
	size_t off = 0;
	for (const Item& it : items)
	{
		if (it.bytes) LSFM_CHECK_HIP(hipMemcpyAsync(P.mem + off, it.src, it.bytes, hipMemcpyDeviceToDevice, ctx->stream));
		*it.dst = it.src ? P.mem + off : nullptr;
		off += (it.bytes + 255) & ~(size_t)255;
	}
	// the factorisation's index arrays are slices of the blob
	const ptrdiff_t shift = (char*)P.ch.blob - (char*)ch.blob;
	auto rebase = [&](int*& p) { if (p) p = (int*)((char*)p + shift); };
	rebase(P.ch.colptr); rebase(P.ch.rowidx); rebase(P.ch.perm); rebase(P.ch.pinv); rebase(P.ch.order); rebase(P.ch.task_cols);
	rebase(P.ch.task_ptr); rebase(P.ch.col_task); rebase(P.ch.col_lpos); rebase(P.ch.col_nin); rebase(P.ch.grp_c0); rebase(P.ch.grp_s);
	rebase(P.ch.grp_nr); rebase(P.ch.col_owner);
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	return sp;
}

// ---- one level ahead ---------------------------------------------------------------------------------------------------------
// What a level that analyses needs from the host -- the pattern of its camera system and the symbolic factorisation --
// depends on index arrays only, and the index arrays of level L + 1's joint maps follow from level L's: the joint map of
// a pair is its two maps side by side (pose pairs inside a map: level L's pattern), plus the hub link of every pose of a
// map the transform re-expresses, plus the pairs across the two maps from the features they share.  So while the device
// factors and refines level L, stream3 puts level L + 1's pattern together from level L's joint maps and the host analyses
// it; level L + 1 finds both waiting and enqueues its factorisation right behind its Schur assembly.
struct PreLevel {
	SchurSystem sy;
	CholSymbolic sym;
	CholHostIn hin;          // what the symbolic analysis reads (kept here: it may run on the helper thread)
	int M = 0;
	HostWorker* worker = nullptr; // non-null: sym is being made there -- wait() before it is read
	// the level's whole plan (counts in ctx->pre_plan): its solve part is completed by the level's solve (pre_plan_complete)
	bool whole = false;
	int level = -1, its = 0;
	void wait()
	{
		HostWorker* w = worker;
		worker = nullptr;
		if (w) w->wait();
	}
	// nothing the helper thread reads goes before the thread is done with it -- whichever path drops the object, exceptions included
	~PreLevel() { try { wait(); } catch (...) {} }
};
void prefetch_next_level(lsfm_context* ctx, const DevBatch& Y, const std::vector<int>& target_ref, int next_level, int step_hint,
                         const unsigned long long* level_keys, int level_nnzb)
{
	ctx->drop_prepared();
	if (!Y.M || Y.B < 2) return;
	// the next level's systems (pairs of Y's maps): small enough for the one-launch dense path?  Then it needs no pattern and no
	// symbolic factorisation, only -- to be enqueued without a host round trip -- its counts
	int most_next = 0;
	for (int b = 0; b < Y.B; b += 2) most_next = std::max(most_next, Y.pose_off[std::min(b + 2, Y.B)] - Y.pose_off[b]);
	const bool next_small = small_level_strips(ctx, most_next) > 0;
	// with the step count an earlier run left for that level, the level can run like a planned one (no round trip at all): then
	// its counts are prepared too.  (LSFM_CHECK_EARLY_PATTERN keeps to the path that compares the pattern.)
	const bool whole = step_hint > 0 && !getenv("LSFM_CHECK_EARLY_PATTERN");
	if (next_small && !whole) return; // (nothing to prepare: the level reads its counts back itself)
	ctx->mark("pre_start");
	auto pl = std::make_shared<PreLevel>();
	pl->M = Y.M;
	Arena& sa = ctx->sarena[next_level & 1];
	sa.reset();
	std::vector<int> counts;
	LevelIndex kept;
	bool ok = false;
	{
		// The joint maps' index arrays are final at evY: the pattern kernels start there, beside the level's right-hand-side kernels and
		// K9.  Measured alternative: start them once K9 has left the main stream, beside the factorisation's chain of small
		// launches -- K9 then runs undisturbed (0.66 -> 0.58 ms per level) but the host gets its pattern 0.6 ms later at every level and
		// the next level is enqueued late: 54.5 instead of 50.4 ms per tree.
		Fork side(ctx, ctx->stream3, evY, false, &sa); // (the small arena of the level's parity)
		if (ctx->timeline_on) { (void)hipEventSynchronize(ctx->ord[evY]); ctx->mark("pre_evY"); }
		int* d_tref = ctx->scratch.alloc<int>(Y.B);
		h2d(ctx, d_tref, target_ref.data(), sizeof(int) * (size_t)Y.B);
		ok = schur_pattern_prefetch(ctx, Y, d_tref, level_keys, level_nnzb, pl->sy, whole ? &counts : nullptr, !next_small, whole ? &kept : nullptr);
		if (ok)
		{
			if (!next_small) chol_fetch(ctx, pl->sy, Y.pose_origin, pl->hin); // (synchronises stream3: the counts have arrived too)
			side.done(evP); // (the next level waits for it: level_plan, level_structure case 3)
		}
	}
	ctx->mark("pre_pat");
	if (!ok) return;
	if (!next_small)
	{
		// The symbolic factorisation is host work that only the level's FACTORISATION needs: it goes to the helper thread, and the
		// caller enqueues the next level's transform, join and Schur assembly meanwhile -- they need the counts only, which arrived
		// with the pattern.  (Done here, on this thread, the device sat idle 1-3 ms at every level boundary waiting for the next
		// level to be enqueued: 9 of an analysing run's 50 ms.)
		if (!ctx->worker) ctx->worker.reset(new HostWorker());
		PreLevel* raw = pl.get(); // (alive until its wait() has returned: ~PreLevel)
		ctx->worker->run([raw]() { chol_symbolic(raw->hin.keys.data(), raw->sy.nnzb, raw->hin.origin.data(), raw->sy.M, raw->sym); });
		pl->worker = ctx->worker.get();
		ctx->mark("pre_sym");
		pl->whole = whole; pl->level = next_level; pl->its = step_hint;
		ctx->pre = pl;
	}
	if (!whole) return;
	// the whole plan of the level: the counts as the host read them now.  A small level's plan is its counts -- its solve is one launch
	// that asks the host nothing; a sparse level's solve part (index arrays of the factorisation to the device) is completed by the
	// level's solve_batch -> pre_plan_complete
	const int B = Y.B;
	ctx->pre_plan.tr_cnt.assign(counts.begin(), counts.begin() + 2 * (B + 1));
	ctx->pre_plan.join_rb.assign(counts.begin() + 2 * (B + 1), counts.end());
	ctx->pre_plan.solve.reset();
	ctx->pre_plan.idx = kept;
	ctx->pre_plan.valid = true;
	ctx->pre_plan_level = next_level;
	ctx->mark("pre_plan");
}
// the solve part of a plan made one level ahead: waits for the symbolic factorisation, sends its index arrays to the device (stream3,
// the small arena of the level's parity) and makes the main stream wait for them
static std::shared_ptr<SolvePlan> pre_plan_complete(lsfm_context* ctx, PreLevel& pl)
{
	pl.wait();
	auto sp = std::make_shared<SolvePlan>();
	sp->sy = pl.sy;
	sp->its = pl.its; sp->mixed = ctx->pcg.mixed; sp->rel_tol = ctx->pcg.rel_tol;
	{
		Fork side(ctx, ctx->stream3, &ctx->sarena[pl.level & 1]); // (what it sends comes from the host)
		chol_upload_index(ctx, pl.sym, sp->ch);
		side.join(evP);
	}
	return sp;
}

// LSFM_DEBUG_CONV=1: sum and maximum of |a[i]| (what went into a large system and what its factorisation left)
__global__ void k_dbg_absstats(size_t n, const double* __restrict__ a, double* __restrict__ out)
{
	double s = 0.0, m = 0.0;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
	{
		const double v = fabs(a[i]);
		s += v; if (v > m || !(v == v)) m = v == v ? v : 1e300;
	}
	atomic_add_f64(out, s);
	atomicMax(reinterpret_cast<unsigned long long*>(out + 1), (unsigned long long)__double_as_longlong(m));
}
// LSFM_DEBUG_CONV=1: the columns whose diagonal factor has an inverse beyond 1e3
__global__ void k_dbg_dinv(int M, const double* __restrict__ Dinv, const double* __restrict__ diag0, const int* __restrict__ colptr, int first_group_col)
{
	int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= M) return;
	double m = 0.0;
	for (int q = 0; q < 36; q++) m = fmax(m, fabs(Dinv[(size_t)j * 36 + q]));
	if (m > 1e3 || !(m == m))
		printf("[lsfm conv] column %d (%s, %d blocks): max |Dinv| %.3e, Dinv diag %.3e %.3e %.3e %.3e %.3e %.3e, diag0 %.3e %.3e %.3e %.3e %.3e %.3e\n", j,
		       j >= first_group_col ? "group" : "leaf", colptr[j + 1] - colptr[j], m, Dinv[(size_t)j * 36], Dinv[(size_t)j * 36 + 7], Dinv[(size_t)j * 36 + 14],
		       Dinv[(size_t)j * 36 + 21], Dinv[(size_t)j * 36 + 28], Dinv[(size_t)j * 36 + 35], diag0[j * 6], diag0[j * 6 + 1], diag0[j * 6 + 2], diag0[j * 6 + 3],
		       diag0[j * 6 + 4], diag0[j * 6 + 5]);
}
// LSFM_FACTOR_DIGEST=1: order-independent digest of an array of 8-byte words (a sum modulo 2^64 of position-mixed bit patterns)
__global__ void k_digest(size_t n, const unsigned long long* __restrict__ a, unsigned long long* out)
{
	unsigned long long h = 0;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
	{
		unsigned long long b = a[i];
		if (b == 0x8000000000000000ull) b = 0; // (-0.0 == 0.0)
		b ^= b >> 31; b *= 0x9E3779B97F4A7C15ull * (2 * (unsigned long long)i + 1); b ^= b >> 29;
		h += b;
	}
	atomicAdd(out, h);
}
__global__ void k_digest_compare(const unsigned long long* d, int* mismatch)
{
	if (d[0] != d[1]) atomicAdd(mismatch, 1);
}
__global__ void k_chol_err_to_run(const int* err, RunStatsDev* run)
{
	if (*err && !run->chol_err) run->chol_err = *err;
}

// The structure of a level on the sparse pipeline, from wherever the level gets it: the camera system with its values assembled, the
// factorisation ready to be scattered into (ch.d_err zeroed).
struct LevelStructure {
	SchurSystem sy;
	CholDev ch;
	SolvePlan* sp = nullptr; // the level's plan (recorded by an earlier run of the tree, or made one level ahead); null: the level analysed
	double tw0 = 0, tw1 = 0; // host clock around the analysis (LSFM_DEBUG)
};
static double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// sp: the plan an earlier run recorded (null: none); pre: what was prepared one level ahead (null: nothing), pending: it is this
// level's whole plan, whose symbolic factorisation may still be under way on the helper thread
static LevelStructure level_structure(lsfm_context* ctx, const SolveIO& io, SolvePlan* sp, PreLevel* pre, bool pending, hipEvent_t eb)
{
	hipStream_t s = ctx->stream;
	LevelStructure ls;
	SchurSystem& sy = ls.sy;
	CholDev& ch = ls.ch;
	// K9 behind the pattern; the chain of the factorisation starts behind it
	auto assemble = [&]() {
		build_schur_values(ctx, io, sy);
		LSFM_REC_T(eb, s); if (roctx().mark) roctx().mark("lsfm factor + refine: begin");
	};
	if (sp || pending)
	{
		// 1. a recorded plan / 2. a plan made one level ahead: the Schur assembly needs the pattern only, so it is enqueued before
		// the host waits for the helper thread
		sy = pending ? pre->sy : sp->sy;
		schur_vinv(ctx, io, sy);
		assemble();
		if (pending)
		{
			ctx->mark("k9_enq");
			ctx->plan->solve = pre_plan_complete(ctx, *pre);
			sp = ctx->plan->solve.get();
			ctx->mark("sym_wait");
		}
		ls.sp = sp;
		ch = sp->ch;
		chol_alloc_values(ctx, ch);
		return ls;
	}
	// the level analyses: pattern -> (copy it to the host) -> numeric assembly K9 enqueued -> symbolic factorisation on the host
	// while K9 runs -> numeric factorisation
	schur_vinv(ctx, io, sy);
	CholHostIn hin;
	bool have = false;
	if (pre && !(pre->M == io.M && !ctx->comm)) pre = nullptr; // (not this level's: dropped by the caller)
	if (pre)
	{
		// 3. prepared while the level below was being solved: pattern (device) and symbolic factorisation (host)
		schur_pattern_early_drop(ctx);
		SchurSystem prepared = pre->sy; // the index members; V^-1 and its factor are this level's (schur_vinv above)
		prepared.IV = sy.IV; prepared.LY = sy.LY; prepared.ymax = sy.ymax; prepared.uu = sy.uu;
		sy = prepared;
		have = true;
		wait_for(ctx, s, evP);
		if (getenv("LSFM_CHECK_EARLY_PATTERN")) schur_pattern_check(ctx, io, sy, "prefetched");
	}
	else if (ctx->early && !ctx->comm)
	{
		// 4. the pattern was put together on stream3 from the level's inputs while the transform ran (a Stereo level that
		// analyses): its second half, and the copy of it for the host's analysis, stay there, behind the joint run pointers (evC_runs)
		{
			Fork side(ctx, ctx->stream3, evC_runs, false);
			ctx->mark("sv_start");
			have = schur_pattern_early_finish(ctx, io, sy);
			ctx->mark("pat_fin");
			if (have)
			{
				if (getenv("LSFM_CHECK_EARLY_PATTERN")) schur_pattern_check(ctx, io, sy, "early");
				chol_fetch(ctx, sy, io.d_pose_origin, hin);
				ctx->mark("fetch");
				schur_pattern_early_extras(ctx, sy);
				side.join(evB);
			}
		}
	}
	else if (io.index_arrays_at_evA && !ctx->comm)
	{
		// 5. the pattern depends on index arrays only: the caller marked the point of the main stream where those were complete
		// (evA) and went on to enqueue its right-hand-side kernels -- the pattern is built on the side stream next to them
		Fork side(ctx, ctx->stream2, evA, false);
		build_schur_pattern(ctx, io, sy);
		chol_fetch(ctx, sy, io.d_pose_origin, hin);
		side.join(evB);
		have = true;
	}
	if (!have)
	{
		// 6. in line, on the main stream (a feature-sharded run; an early build whose table overflowed)
		build_schur_pattern(ctx, io, sy);
		chol_fetch(ctx, sy, io.d_pose_origin, hin);
	}
	assemble();
	ls.tw0 = wall_ms();
	ctx->mark("k9_enq");
	if (pre) { pre->wait(); chol_upload_symbolic(ctx, pre->sym, ch); }
	else chol_analyse(ctx, sy, hin, ch);
	ctx->mark("analyse");
	ls.tw1 = wall_ms();
	return ls;
}

// A level of small systems (at most 16 poses each): assembled, factored and solved by one launch (lsfm_small.hip) -- no pattern of S,
// no symbolic factorisation; the level above builds its pattern from its own joint maps when this one leaves none
// (schur_pattern_prefetch / schur_pattern_early_issue).  warm: the level has a recorded plan (SolvePlan::small)
static SolveOutcome solve_level_dense(lsfm_context* ctx, const SolveIO& io, int strips, bool warm, hipEvent_t eb, hipEvent_t ec, hipEvent_t ed)
{
	hipStream_t s = ctx->stream;
	LevelPlan* lp = ctx->plan;
	if (!warm) schur_pattern_early_drop(ctx);
	int* d_small = nullptr; // [2] status of the small path + (as a double behind them) the level's largest relative residual
	auto enqueue = [&]() {
		d_small = ctx->scratch.alloc<int>(4);
		dev_zero(ctx, d_small, 4 * sizeof(int));
		hipEvent_t esm0 = nullptr, esm1 = nullptr;
		if (ctx->stats) { esm0 = ctx->pool_event(); esm1 = ctx->pool_event(); LSFM_REC_T(esm0, s); }
		small_solve_launch(ctx, io, strips, d_small, reinterpret_cast<double*>(d_small + 2));
		if (ctx->stats) { LSFM_REC_T(esm1, s); ctx->defer_time(esm0, esm1, &ctx->stats->t_small_ms); ctx->stats->small_levels++; }
	};
	// (a planned level brackets its launch like a level on the sparse pipeline brackets its factorisation)
	if (!warm) enqueue();
	LSFM_REC_T(eb, s); if (warm && roctx().mark) roctx().mark("lsfm factor + refine: begin");
	if (warm) enqueue();
	LSFM_REC_T(ec, s);
	LSFM_REC_T(ed, s); if (roctx().mark) roctx().mark("lsfm solve: end");
	SolveOutcome oc; // (keys: no pattern left for the level above)
	oc.end = ed;
	oc.steps_used = 1;
	if (ctx->stats) ctx->stats->pcg_iterations += 1;
	// (a plan made one level ahead is the run's own: nothing to record, nothing to stop for)
	const bool deferred = ctx->in_tree_run && ctx->d_run && (warm || !lp || lp == &ctx->pre_plan);
	if (deferred) return oc; // the kernel left its verdict in the run's device record (read at the end of the run)
	int hs[4];
	d2h_ints(ctx, d_small, hs, 4); // synchronises
	if (hs[1]) LSFM_FAIL(LSFM_ERR_NOT_SPD, "Schur system is not positive definite (system " + std::to_string(hs[1] - 1) + " of the level)");
	double mr;
	memcpy(&mr, hs + 2, sizeof mr);
	if (ctx->stats) ctx->stats->max_rel_residual = std::max(ctx->stats->max_rel_residual, mr);
	if (lp && !lp->solve && hs[0] == 0)
	{
		// the plan of a small level: nothing but the fact that it is one (the structure of its solve is the batch's offsets)
		auto small_plan = std::make_shared<SolvePlan>();
		small_plan->its = 1; small_plan->mixed = false; small_plan->rel_tol = ctx->pcg.rel_tol; small_plan->small = true;
		lp->solve = small_plan;
	}
	oc.not_converged = hs[0];
	return oc;
}

// LSFM_FACTOR_DIGEST=1 (tests): digests of S and of the factor into the run's device record, and -- one GPU -- the same system
// assembled and factored a second time: the bits must not depend on the order in which the work-groups land their sums
static void factor_digest_check(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, CholDev& ch)
{
	static const bool digest = getenv("LSFM_FACTOR_DIGEST") != nullptr;
	if (!digest || !ctx->d_run) return;
	hipStream_t s = ctx->stream;
	Arena& sc = ctx->scratch;
	const int M = io.M;
	auto dg = [&](const double* a, size_t n, unsigned long long* out) {
		if (a && n) hipLaunchKernelGGL(k_digest, dim3(256), dim3(256), 0, s, n, reinterpret_cast<const unsigned long long*>(a), out);
	};
	dg(sy.S, (size_t)sy.nnzb * 36, &ctx->d_run->s_digest);
	if (!ctx->comm)
	{
		// the SAME camera systems assembled a second time (U scatter, K9 with all its variants, the fallback kernel): their
		// work-groups land their sums in another order -- the bits of S and E must not depend on it (fixed-point sums,
		// lsfm_schur_panel.hip).  (The stage timings and flop counts of the run count this second assembly too: a debug mode.)
		SchurSystem sy2 = sy;
		build_schur_values(ctx, io, sy2);
		unsigned long long* d = sc.alloc<unsigned long long>(2);
		dev_zero(ctx, d, 2 * sizeof(unsigned long long));
		dg(sy.S, (size_t)sy.nnzb * 36, d); dg(sy.E, (size_t)M * 6, d);
		dg(sy2.S, (size_t)sy.nnzb * 36, d + 1); dg(sy2.E, (size_t)M * 6, d + 1);
		hipLaunchKernelGGL(k_digest_compare, dim3(1), dim3(1), 0, s, d, &ctx->d_run->s_rebuild_mismatch);
	}
	// leaf columns: factored in place in L; group columns: in Lg (their slots of L hold the spent accumulators: integers, summed alike)
	auto factor_digest = [&](unsigned long long* out) {
		dg(ch.Dinv, (size_t)ch.M * 36, out);
		dg(ch.L, (size_t)ch.nnzL * 36, out);
		if (ch.Lg) dg(ch.Lg, (size_t)ch.nnzL * 36, out);
	};
	factor_digest(&ctx->d_run->factor_digest);
	if (!ctx->comm)
	{
		// ... and the SAME system factored a second time (its work-groups will be scheduled differently, the atomics land in another
		// order): the two factors must be the same bits.  d[0], d[1]: the digests of this system's two factors alone
		unsigned long long* d = sc.alloc<unsigned long long>(2);
		dev_zero(ctx, d, 2 * sizeof(unsigned long long));
		factor_digest(d);
		dev_zero(ctx, ch.L, (size_t)ch.nnzL * 36 * sizeof(double));
		if (ch.Lg) dev_zero(ctx, ch.Lg, (size_t)ch.nnzL * 36 * sizeof(double));
		chol_scatter(ctx, sy, io.d_fixed, ch);
		chol_factor(ctx, sy, io.d_fixed, ch, nullptr);
		factor_digest(d + 1);
		hipLaunchKernelGGL(k_digest_compare, dim3(1), dim3(1), 0, s, d, &ctx->d_run->refactor_mismatch);
	}
}

// LSFM_DEBUG_CONV=1: the systems a level leaves above 1e-9; what went into the root system of a large tree and what its
// factorisation and solve left
static void debug_conv(lsfm_context* ctx, const SolveIO& io, const SchurSystem& sy, const CholDev& ch, const PcgSeg* seg)
{
	hipStream_t s = ctx->stream;
	const int M = io.M;
	hipLaunchKernelGGL(k_pcg_debug, dim3((io.nseg + 127) / 128), dim3(128), 0, s, io.nseg, M, seg);
	if (!(M > 10000 && io.nseg == 1)) return;
	double* d = ctx->scratch.alloc<double>(12);
	dev_zero(ctx, d, 12 * sizeof(double));
	auto st = [&](const double* a, size_t n, int k) { if (a && n) hipLaunchKernelGGL(k_dbg_absstats, dim3(512), dim3(256), 0, s, n, a, d + 2 * k); };
	st(sy.S, (size_t)sy.nnzb * 36, 0); st(sy.E, (size_t)M * 6, 1); st(ch.L, (size_t)ch.nnzL * 36, 2); st(ch.Lg, (size_t)ch.nnzL * 36, 3);
	st(ch.Dinv, (size_t)ch.M * 36, 4); st(io.x_pose, (size_t)M * 6, 5);
	hipLaunchKernelGGL(k_dbg_dinv, dim3((ch.M + 255) / 256), dim3(256), 0, s, ch.M, ch.Dinv, ch.diag0, ch.colptr, 0);
	double h[12];
	d2h(ctx, h, d, sizeof h);
	fprintf(stderr, "[lsfm conv] root M=%d: |S| sum %.15e max %.6e  |E| sum %.15e  |L| sum %.12e max %.3e  |Lg| sum %.12e max %.3e  |Dinv| sum %.6e max %.3e  |x| sum %.12e max %.3e\n",
	        M, h[0], h[1], h[2], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11]);
}

// One level's camera systems: the dense path for a level of small systems; otherwise the level's structure, the refinement's set-up,
// the factorisation with the first forward substitution riding on it, the refinement, the back-substitution, and the outcome --
// left in the run's device record, or read here and, for a level that converged, kept with its structure as the level's plan
SolveOutcome solve_batch(lsfm_context* ctx, const SolveIO& io)
{
	hipStream_t s = ctx->stream;
	const int M = io.M;
	LevelPlan* lp = ctx->plan;
	const int strips = (io.d_pose_off && io.d_feat_off && io.d_u_off) ? small_level_strips(ctx, io.seg_rows) : 0;
	SolvePlan* sp = lp ? lp->solve.get() : nullptr;
	// (a plan recorded on the other path -- lsfm_set_small_solve was changed between two runs of a resident tree -- is void)
	if (sp && sp->small != (strips > 0)) { lp->solve.reset(); sp = nullptr; }
	// what was prepared one level ahead leaves the context here; wherever it is dropped, its release waits for the helper thread.
	// pending: it is this level's whole plan, whose symbolic factorisation may still be under way there
	std::shared_ptr<PreLevel> pre = std::move(ctx->pre);
	const bool pending = !strips && !sp && pre && pre->whole && lp == &ctx->pre_plan;
	if (pre && !pending && (strips || sp || pre->whole || pre->M != M || ctx->comm)) pre.reset(); // (not this level's, or of no use to it)
	const bool warm = sp != nullptr || pending; // pattern + symbolic factorisation known from an earlier run of the same tree level (or made one level ahead)
	hipEvent_t ea = ctx->pool_event(), eb = ctx->pool_event(), ec = ctx->pool_event(), ed = ctx->pool_event();
	LSFM_REC_T(ea, s); if (roctx().mark) roctx().mark("lsfm schur: begin");
	if (strips) return solve_level_dense(ctx, io, strips, warm, eb, ec, ed);
	LevelStructure ls = level_structure(ctx, io, sp, pre.get(), pending, eb);
	pre.reset();
	const SchurSystem& sy = ls.sy;
	CholDev& ch = ls.ch;
	sp = ls.sp;
	const bool dbg = getenv("LSFM_DEBUG") != nullptr;
	PcgWork w = pcg_begin(ctx, io, sy, ch);
	if (ctx->stats && chol_distributed(ctx, ch)) { ctx->stats->dist_solves++; ctx->stats->dist_work_total += ch.work_total; ctx->stats->dist_work_shared += ch.work_shared; }
	chol_scatter(ctx, sy, io.d_fixed, ch);
	if (w.fused_fwd) chol_perm_in(ctx, ch, w.r, io.d_fixed, w.v);
	chol_factor(ctx, sy, io.d_fixed, ch, w.fused_fwd ? w.v : nullptr);
	if (ctx->pcg.mixed) chol_round_to_float(ctx, ch);
	factor_digest_check(ctx, io, sy, ch);
	if (dbg) { LSFM_CHECK_HIP(hipStreamSynchronize(s)); }
	const double tw2 = wall_ms();
	// inside a tree run the outcome of a level (a non-positive pivot, systems left above their bound, the largest residual) is
	// left in the run's device record and read once at the end of the run; a stage-level call, and a level whose structure is
	// being recorded as a plan, reads it here
	const bool deferred = warm || (ctx->in_tree_run && ctx->d_run && !lp);
	const PcgSteps steps{ warm, deferred, sp ? sp->its : 0, sp ? sp->mixed : false, sp ? sp->rel_tol : 0.0 };
	const PcgResult res = pcg_run(ctx, io, sy, ch, w, steps);
	if (dbg)
	{
		LSFM_CHECK_HIP(hipStreamSynchronize(s));
		fprintf(stderr, "[lsfm] solve M=%d nseg=%d nnzb=%d nnzL=%d etree levels=%d tail=%d leaf tasks=%d group levels=%d %s| analyse %.2f ms, factor %.2f ms, cg(%d its) %.2f ms\n", M, io.nseg,
		        sy.nnzb, ch.nnzL, ch.nlevels, ch.M - ch.tail_begin, ch.ntask0, (int)ch.glevel_ptr.size() - 1, warm ? "(plan) " : "", ls.tw1 - ls.tw0, tw2 - ls.tw1, res.its, wall_ms() - tw2);
	}
	if (ctx->comm)
	{
		// feature-sharded run: every rank solved the same system, but the factorisations add their updates in whatever order the
		// atomics land -- the solutions may differ in the last bit.  Rank 0's replaces everyone's, so that the replicated state
		// (and every decision taken from it) stays the same on all ranks.
		Comm& cm = *ctx->comm;
		const size_t nscal = (size_t)M * 6;
		double *x = io.x_pose, *xb = cm.alloc<double>(nscal);
		if (cm.rank == 0) LSFM_CHECK_HIP(hipMemcpyAsync(xb, x, nscal * sizeof(double), hipMemcpyDeviceToDevice, s));
		else fill_async(s, xb, 0, nscal * sizeof(double));
		cm.allreduce(s, xb, nscal, LSFM_DTYPE_F64);
		LSFM_CHECK_HIP(hipMemcpyAsync(x, xb, nscal * sizeof(double), hipMemcpyDeviceToDevice, s));
	}
	pcg_final_residual(ctx, io, sy, w); // (nothing here waits for the device before the back-substitution is enqueued)
	LSFM_REC_T(ec, s); if (roctx().mark) roctx().mark("lsfm back-substitution: begin");
	launch_backsub(ctx, io, sy, io.x_pose);
	LSFM_CHECK_HIP(hipGetLastError());
	LSFM_REC_T(ed, s); if (roctx().mark) roctx().mark("lsfm solve: end");
	SolveOutcome oc;
	oc.keys = sy.upper_keys; oc.nnzb = sy.nnzb;
	oc.end = ed;
	if (ctx->stats)
	{
		lsfm_stats* st = ctx->stats;
		ctx->defer_time(ea, eb, &st->t_schur_ms);
		ctx->defer_time(eb, ec, &st->t_pcg_ms);
		ctx->defer_time(ec, ed, &st->t_backsub_ms);
		ctx->defer_time(w.es0, w.es1, &st->spmv_ms);
		st->pcg_iterations += res.its;
		st->spmv_launches += 1; // (the one product that was timed)
		st->spmv_bytes += spmv_bytes(sy);
		st->spmv_nnzb_upper_last = sy.nnzb; st->spmv_rows_last = M;
	}
	oc.steps_used = res.planned ? 0 : std::max(res.its, 1);
	if (deferred)
	{
		if (warm && !res.planned) { sp->its = std::max(res.its, 1); sp->mixed = ctx->pcg.mixed; sp->rel_tol = ctx->pcg.rel_tol; } // precision / tolerance changed: the count was re-learnt
		static const bool dbg_conv = getenv("LSFM_DEBUG_CONV") != nullptr;
		if (dbg_conv) debug_conv(ctx, io, sy, ch, w.seg);
		hipLaunchKernelGGL(k_pcg_run_stats, dim3((io.nseg + 127) / 128), dim3(128), 0, s, io.nseg, w.seg, ctx->d_run);
		return oc; // the outcome is read at the end of the run (lsfm_tree_run)
	}
	double maxrel = 0;
	int notconv = pcg_read_verdict(ctx, io, w, &maxrel); // synchronises
	if (ctx->stats) ctx->stats->max_rel_residual = std::max(ctx->stats->max_rel_residual, maxrel);
	if (ctx->comm)
	{
		// feature-sharded run: the verdict (and with it whether this level keeps a plan, i.e. whether the NEXT run of the level is
		// warm) must be the same on every rank -- a rank that is cold alone would issue pattern all-reduces nobody joins.  Every
		// rank solved the same system; the residuals they computed differ in the last bit at most, but a count taken at a
		// threshold may: summed over the ranks, any rank's doubt is everybody's.
		long long hv[2] = { notconv, 0 };
		comm_sum_host(ctx, hv, 2);
		notconv = (int)((hv[0] + ctx->comm->world - 1) / ctx->comm->world);
	}
	// what depends on the structure only stays with the tree level for its next runs
	if (lp && !lp->solve && notconv == 0) lp->solve = solve_plan_store(ctx, sy, ch, std::max(res.its, 1));
	oc.not_converged = notconv;
	return oc;
}

} // namespace lsfm
